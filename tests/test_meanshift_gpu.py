"""GPU tests of the device MeanShift (catgrasp_amd/cluster.py, csrc/meanshift.hip) and of the scene-to-objects step built on it.

Yardsticks: scikit-learn 1.7.2's recorded results on the golden scenes (tests/golden/meanshift_golden.npz; the generator admits a
scene only if float32 and float64 input give scikit-learn the same labels and no point or center order sits on a knife-edge), and
tests/meanshift_ref.py, the float64 restatement of the kernels' arithmetic (proved against scikit-learn in
tests/test_meanshift_ref_cpu.py, which also shows that the summation order changes no count on these scenes).

Bounds: labels, number and order of centers, n_iter_, per-seed counts and iterations are EQUAL.  Centers are within
stop_thresh = 1e-3 * bandwidth of scikit-learn's (two converged climbs may stop that far apart).  Per-seed means are within 1e-12 m
of the restatement's: float64 summation-order noise for a few thousand coordinates below 1 m is ~1e-16 * sqrt(n) ~ 1e-14 m per
iteration, and the scenes have no membership knife-edge through which it could grow."""
import numpy as np
import pytest
import torch

import meanshift_ref as ref
from catgrasp_amd import cluster, pipeline, segmentation

pytestmark = pytest.mark.gpu


def _X(name, dtype):
    X, bw = ref.scene(name)
    return X.astype(dtype), bw


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
@pytest.mark.parametrize('name', ref.scenes())
def test_meanshift_matches_scikit_learn(name, dtype, cuda_device):
    """Through cluster.MeanShift, for the float32 scene and for the same values as float64 (for `streamed` the float64 run is the
    streamed route at its smallest size; scikit-learn's labels are the same for both by the generator's condition 1)."""
    g = ref.golden()
    X, bw = _X(name, dtype)
    ms = cluster.MeanShift(bandwidth=bw, cluster_all=True, n_jobs=-1, seeds=None)
    labels = ms.fit_predict(X)
    want = g[f'{name}_centers_f64']
    assert ms.cluster_centers_.dtype == np.float64 and ms.cluster_centers_.shape == want.shape
    gap = np.abs(ms.cluster_centers_ - want).max()
    print(f'{name} {dtype}: n {len(X)} centers {len(want)} n_iter {ms.n_iter_} center gap to scikit-learn {gap:.3g} m (stop_thresh {1e-3 * bw:.3g} m)')
    assert labels.dtype == np.int64 and labels is ms.labels_
    assert np.array_equal(labels, g[f'{name}_labels_{"f32" if dtype == "float32" else "f64"}'])
    assert gap <= 1e-3 * bw
    assert ms.n_iter_ == int(g[f'{name}_n_iter_f64'])


@pytest.mark.parametrize('name', ref.scenes())
def test_climb_matches_the_restatement_per_seed(name, cuda_device):
    X, bw = ref.scene(name)
    r = ref.reference(name)
    pts = torch.from_numpy(X).to(cuda_device)
    means, counts, iters = cluster.climb(pts, pts.double(), bw)
    assert np.array_equal(counts.cpu().numpy(), r['counts']) and np.array_equal(iters.cpu().numpy(), r['iters'])
    gap = np.abs(means.cpu().numpy() - r['means']).max()
    print(f'{name}: largest per-seed mean gap to the restatement {gap:.3g} m')
    assert gap <= 1e-12
    centers = cluster.merge(cluster.sort_centers(means, counts), bw).cpu().numpy()
    assert centers.shape == r['centers'].shape and np.abs(centers - r['centers']).max() <= 1e-12


def test_two_runs_are_bitwise_identical(cuda_device):
    X, bw = ref.scene('touching')
    pts = torch.from_numpy(X).to(cuda_device)
    a, b = cluster.climb(pts, pts.double(), bw), cluster.climb(pts, pts.double(), bw)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    m1, m2 = cluster.MeanShift(bw).fit(X), cluster.MeanShift(bw).fit(X)
    assert np.array_equal(m1.labels_, m2.labels_) and m1.cluster_centers_.tobytes() == m2.cluster_centers_.tobytes()


@pytest.mark.parametrize('dtype', ['float32', 'float64'])
def test_lds_and_streamed_routes_are_bitwise_identical(dtype, cuda_device):
    X, bw = _X('nut', dtype)
    pts = torch.from_numpy(X).to(cuda_device)
    lds, streamed = cluster.climb(pts, pts.double(), bw, route='lds'), cluster.climb(pts, pts.double(), bw, route='streamed')
    assert all(torch.equal(u, v) for u, v in zip(lds, streamed))
    a, b = cluster.MeanShift(bw, _route='lds').fit(X), cluster.MeanShift(bw, _route='streamed').fit(X)
    assert np.array_equal(a.labels_, b.labels_) and a.cluster_centers_.tobytes() == b.cluster_centers_.tobytes()
    # the LDS route refuses a cloud it cannot hold instead of reading past its allocation
    big = torch.zeros((160 * 1024 // pts.element_size() // 3 + 1, 3), dtype=pts.dtype, device=cuda_device)
    with pytest.raises(cluster.L.CatgraspAmdError):
        cluster.climb(big, big[:1].double().contiguous(), bw, route='lds')


def test_the_result_does_not_depend_on_how_seeds_are_spread_over_waves(cuda_device):
    """A seed climbed alone (one wave, one workgroup) ends where it ends among 1,680 others."""
    X, bw = ref.scene('nut')
    pts = torch.from_numpy(X).to(cuda_device)
    full = cluster.climb(pts, pts.double(), bw)
    for lo, hi in ((0, 1), (5, 22), (1000, 1680)):
        part = cluster.climb(pts, pts[lo:hi].double().contiguous(), bw)
        assert all(torch.equal(u[lo:hi], v) for u, v in zip(full, part))


def test_float64_input_and_device_tensors(cuda_device):
    X, bw = ref.scene('screw')
    a = cluster.MeanShift(bw).fit(X)
    b = cluster.MeanShift(bw).fit(torch.from_numpy(X.astype(np.float64)).to(cuda_device))
    assert np.array_equal(a.labels_, b.labels_) and a.cluster_centers_.tobytes() == b.cluster_centers_.tobytes()


def test_explicit_seeds_match_the_restatement(cuda_device):
    X, bw = ref.scene('nut')
    seeds = X[::7]
    r = ref.mean_shift(X, bw, seeds=seeds)
    ms = cluster.MeanShift(bw, seeds=seeds).fit(X)
    assert np.array_equal(ms.labels_, r['labels']) and ms.n_iter_ == r['n_iter']
    assert ms.cluster_centers_.shape == r['centers'].shape and np.abs(ms.cluster_centers_ - r['centers']).max() <= 1e-12
    # seeds in empty space only: scikit-learn's error
    with pytest.raises(ValueError, match='No point was within bandwidth'):
        cluster.MeanShift(bw, seeds=np.array([[5.0, 5.0, 5.0]])).fit(X)
    # one empty seed among good ones is dropped, and still counts for n_iter_ like any seed
    mixed = cluster.MeanShift(bw, seeds=np.concatenate([seeds, [[5.0, 5.0, 5.0]]])).fit(X)
    assert np.array_equal(mixed.labels_, ms.labels_) and mixed.cluster_centers_.tobytes() == ms.cluster_centers_.tobytes()


def test_max_iter_caps_the_climb(cuda_device):
    X, bw = ref.scene('touching')
    r = ref.climb(X, X, bw, max_iter=3)
    pts = torch.from_numpy(X).to(cuda_device)
    means, counts, iters = cluster.climb(pts, pts.double(), bw, max_iter=3)
    assert int(iters.max()) == 3 and np.array_equal(iters.cpu().numpy(), r[2]) and np.array_equal(counts.cpu().numpy(), r[1])
    assert np.abs(means.cpu().numpy() - r[0]).max() <= 1e-12


def test_cluster_all_false_marks_a_far_outlier(cuda_device):
    X, bw = ref.scene('tiny')
    base = cluster.MeanShift(bw).fit(X)
    Xo = np.concatenate([X, X[:1] + np.float32(0.5)])
    # seeds = the scene's own points, so the outlier founds no center of its own
    strict = cluster.MeanShift(bw, seeds=X, cluster_all=False).fit(Xo)
    loose = cluster.MeanShift(bw, seeds=X, cluster_all=True).fit(Xo)
    assert strict.labels_[-1] == -1 and loose.labels_[-1] >= 0
    assert np.array_equal(loose.labels_[:-1], base.labels_)
    inside = np.linalg.norm(X.astype(np.float64) - base.cluster_centers_[base.labels_], axis=1) <= bw
    assert np.array_equal(strict.labels_[:-1], np.where(inside, base.labels_, -1)) and inside.mean() > 0.9


def test_predict_and_input_refusals(cuda_device):
    X, bw = ref.scene('tiny')
    ms = cluster.MeanShift(bw).fit(X)
    new = (ms.cluster_centers_[[2, 0, 3, 1, 1]] + 0.001).astype(np.float32)
    assert ms.predict(new).tolist() == [2, 0, 3, 1, 1] and ms.predict(new).dtype == np.int64
    assert np.array_equal(ms.predict(X), ms.labels_)
    bad = X.copy()
    bad[3, 1] = np.nan
    with pytest.raises(ValueError):
        cluster.MeanShift(bw).fit(bad)
    with pytest.raises(ValueError):
        cluster.MeanShift(bw, seeds=np.array([[0.0, np.inf, 0.0]])).fit(X)
    with pytest.raises(ValueError):
        cluster.MeanShift(bw).fit(X[:, :2])


# ---- the scene-to-objects step on a synthetic bin ----

PLATE = np.array([0.020, 0.012, 0.002])
SIZES = (2400, 2100, 1800, 1500, 1200, 900, 700, 300)          # eight plates; the last is the planted too-small object
SPARSE = 600                                                   # points of the planted sparse cluster, spread over a 6 cm cube


def _bin():
    rng = np.random.default_rng(11)
    xyz, planted, centers = [], [], []
    for k, n in enumerate(SIZES):
        c = np.array([(k % 3) * 0.04, (k // 3) * 0.04, 0.6])
        xyz.append(c + (rng.uniform(0, 1, (n, 3)) - 0.5) * PLATE)
        planted.append(np.full(n, k)); centers.append(c)
    c = np.array([-0.15, 0.0, 0.6])
    xyz.append(c + (rng.uniform(0, 1, (SPARSE, 3)) - 0.5) * 0.06)
    planted.append(np.full(SPARSE, len(SIZES))); centers.append(c)
    perm = rng.permutation(sum(SIZES) + SPARSE)
    xyz, planted = np.concatenate(xyz)[perm], np.concatenate(planted)[perm]
    original = xyz.astype(np.float32)                          # the network's input points: the cloud in float32
    offsets = (0.9 * (np.array(centers)[planted] - original) + rng.normal(0, 0.0002, xyz.shape)).astype(np.float32)
    normals = rng.normal(size=xyz.shape)
    return xyz, normals, original, offsets, planted


def test_scene_to_objects_on_a_synthetic_bin(cuda_device):
    xyz, normals, original, offsets, planted = _bin()
    labels = segmentation.instances_from_offsets(xyz, original, offsets, class_name='nut')
    assert labels.shape == planted.shape and labels.dtype == np.int64
    shifted = segmentation.instances_from_offsets.xyz_shifted
    assert shifted.dtype == np.float32 and shifted.shape[1] == 3 and len(shifted) < len(xyz)
    # the recovered partition is the planted one: one label per planted object, nine different labels
    first = {k: int(labels[planted == k][0]) for k in range(len(SIZES) + 1)}
    assert len(set(first.values())) == len(SIZES) + 1
    assert np.array_equal(labels, np.array([first[k] for k in range(len(SIZES) + 1)])[planted])
    # MeanShift numbers its clusters by intensity, and the given bandwidth overrides the class table
    assert np.array_equal(segmentation.instances_from_offsets(xyz, original, offsets, bandwidth=0.007), labels)

    cleaned, order = segmentation.select_segments(torch.from_numpy(xyz).to(cuda_device), torch.from_numpy(labels).to(cuda_device))
    assert np.array_equal(cleaned, np.where(planted >= len(SIZES) - 1, -1, labels))          # the 300-point plate and the sparse cluster go
    assert order.tolist() == [first[k] for k in range(len(SIZES) - 1)]                       # the rest, largest first
    cpu_cleaned, cpu_order = segmentation.select_segments(xyz, labels)
    assert np.array_equal(cpu_cleaned, cleaned) and np.array_equal(cpu_order, order)

    objects = pipeline.objects_from_segmentation(xyz, normals, cleaned, order)
    assert [len(o['ob_pts']) for o in objects] == list(SIZES[:-1])
    for k, o in enumerate(objects):
        assert np.array_equal(o['ob_pts'], xyz[planted == k]) and np.array_equal(o['ob_normals'], normals[planted == k])
    assert sum(len(o['ob_pts']) for o in objects) == int((cleaned >= 0).sum())
