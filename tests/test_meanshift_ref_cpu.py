"""CPU proof of tests/meanshift_ref.py, the float64 restatement that tests/test_meanshift_gpu.py holds the device kernels to: on every
golden scene it reproduces scikit-learn 1.7.2 (tests/golden/meanshift_golden.npz), and the order in which it visits the points does
not change a single count or iteration number -- the scenes sit on no membership knife-edge, which is what lets the device, whose
sums run in yet another order, be held to equality."""
import numpy as np
import pytest

import meanshift_ref as ref


@pytest.mark.parametrize('name', ref.scenes())
def test_restatement_reproduces_scikit_learn(name):
    g, (X, bw) = ref.golden(), ref.scene(name)
    r = ref.reference(name)
    assert np.array_equal(r['labels'], g[f'{name}_labels_f64']) and np.array_equal(r['labels'], g[f'{name}_labels_f32'])
    assert r['centers'].shape == g[f'{name}_centers_f64'].shape
    assert r['n_iter'] == int(g[f'{name}_n_iter_f64']) == int(g[f'{name}_n_iter_f32'])
    gap = np.abs(r['centers'] - g[f'{name}_centers_f64']).max()
    print(f'{name}: center gap to scikit-learn (f64) {gap:.3g} m, stop_thresh {1e-3 * bw:.3g} m')
    assert gap <= 1e-3 * bw


@pytest.mark.parametrize('name', ref.scenes())
def test_point_order_changes_no_count_and_no_iteration_number(name):
    X, bw = ref.scene(name)
    r = ref.reference(name)
    means, counts, iters = ref.climb(X[::-1], X, bw)
    assert np.array_equal(counts, r['counts']) and np.array_equal(iters, r['iters'])
    assert np.abs(means - r['means']).max() <= 1e-12


def test_golden_scenes_cover_the_wave_boundary_and_the_streamed_route():
    n = {s: len(ref.scene(s)[0]) for s in ref.scenes()}
    assert n['one'] == 1 and (n['wave63'], n['wave64'], n['wave65']) == (63, 64, 65)
    assert n['streamed'] * 24 > 160 * 1024 >= (n['streamed'] - 4) * 24          # a few more f64 points than the LDS route takes
    assert int(ref.golden()['touching_n_iter_f64']) >= 29                       # the long, divergent climbs


def test_stop_rule_on_hand_cases():
    X = np.array([[0, 0, 0], [0.004, 0, 0], [1, 0, 0]], dtype=np.float64)
    # seed 0 sees both near points: mean 0.002 (moved 0.002 > 1e-5) -> 1 completed; the next mean is the same -> stop
    means, counts, iters = ref.climb(X, X[:1], 0.01)
    assert np.allclose(means, [[0.002, 0, 0]]) and counts.tolist() == [2] and iters.tolist() == [1]
    # max_iter = 0: one query, no completed iteration;  a seed with no point in reach is empty and keeps its place
    means, counts, iters = ref.climb(X, np.array([[0, 0, 0], [0.5, 0, 0]]), 0.01, max_iter=0)
    assert counts.tolist() == [2, 0] and iters.tolist() == [0, 0] and means[1].tolist() == [0.5, 0, 0]
    # membership is <=: a point at exactly the bandwidth is inside
    assert ref.climb(np.array([[0.25, 0, 0]]), np.array([[0.0, 0, 0]]), 0.25, max_iter=0)[1].tolist() == [1]


def test_merge_order_and_suppression_on_a_hand_case():
    means = np.array([[0, 0, 0], [0.05, 0, 0], [0.2, 0, 0], [0.2, 0, 0.01], [0.1, 0, 0]])
    counts = np.array([5, 9, 7, 7, 0])
    centers, k = ref.merge(means, counts, 0.06)
    # (9, 0.05) first and kills (5, 0); of the two sevens the larger tuple, z = 0.01, leads and kills the other; the empty seed is dropped
    assert centers.tolist() == [[0.05, 0, 0], [0.2, 0, 0.01]] and k.tolist() == [9, 7]
