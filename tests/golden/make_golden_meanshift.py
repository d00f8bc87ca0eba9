"""Regenerates tests/golden/meanshift_golden.npz with scikit-learn 1.7.2, the library the reference calls
(predicter.py:332).  Run from the repository root on a host with scikit-learn:  python tests/golden/make_golden_meanshift.py

Every scene is seeded and synthetic: Gaussian blobs ("objects") whose points are the contracted, shifted coordinates that the
clustering sees, stored float32 and shuffled.  Per scene the file holds X, the bandwidth, and scikit-learn's labels_,
cluster_centers_ and n_iter_ for the float32 array and for the same values as float64.

A scene is written only if it is a fair yardstick for an implementation that computes in float64 with another summation order:
  1. the float32-input and float64-input runs give identical labels_ and n_iter_;
  2. their centers differ by less than 0.1 * stop_thresh (stop_thresh = 1e-3 * bandwidth);
  3. every point is nearer to its center than to the second-nearest by at least 50 * stop_thresh;
  4. the kept centers' intensities (sizes of their last radius query) differ pairwise by at least 5 points;
  5. the whole file is no larger than the largest golden already committed.
A scene that fails one raises: change its seed."""
import os
import sys
import time

import numpy as np
import sklearn
from sklearn.cluster import MeanShift

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..'))
import meanshift_ref  # noqa: E402

OUT = os.path.join(HERE, 'meanshift_golden.npz')
PITCH, DEPTH = 0.03, 0.6
F64_LDS_POINTS = 160 * 1024 // 24          # the seed climb stages f64 points in LDS up to this count (csrc/meanshift.hip)


def blobs(seed, sizes, sigma, centers=None):
    rng = np.random.default_rng(seed)
    if centers is None:                     # a grid at about 3 cm pitch, jittered by 2 mm
        side = int(np.ceil(np.sqrt(len(sizes))))
        centers = np.array([[(i % side) * PITCH, (i // side) * PITCH, DEPTH] for i in range(len(sizes))])
        centers = centers + rng.normal(0, 0.002, centers.shape)
    pts = np.concatenate([c + rng.normal(0, 1, (n, 3)) * np.asarray(sigma) for c, n in zip(centers, sizes)])
    return rng.permutation(pts).astype(np.float32)


def touching(seed, sizes):
    rng = np.random.default_rng(seed)
    centers = np.concatenate([rng.uniform(0, 0.04, (len(sizes), 2)), np.full((len(sizes), 1), DEPTH)], axis=1)
    return blobs(seed + 1, sizes, (0.006, 0.002, 0.002), centers)


SCENES = {
    'one': (lambda: np.array([[0.01, 0.02, DEPTH]], dtype=np.float32), 0.005),
    'wave63': (lambda: blobs(63, (40, 23), 0.0008), 0.005),
    'wave64': (lambda: blobs(64, (40, 24), 0.0008), 0.005),
    'wave65': (lambda: blobs(65, (40, 25), 0.0008), 0.005),
    'tiny': (lambda: blobs(1, (70, 45, 20, 9), 0.001), 0.005),
    'nut': (lambda: blobs(2, (400, 330, 270, 220, 170, 130, 100, 60), (0.003, 0.0015, 0.0015)), 0.007),
    'screw': (lambda: blobs(6, (700, 600, 500, 400, 300), (0.0045, 0.002, 0.0015)), 0.009),
    'touching': (lambda: touching(10, (420, 360, 310, 280, 240, 190)), 0.007),
    # a few more f64 points than fit in LDS: run with float64 input this is the streamed route at its smallest size
    'streamed': (lambda: blobs(5, (1000, 930, 860, 790, 720, 650, 580, 510, 440, 350), 0.001), 0.007),
}


def run(X, bw):
    t0 = time.perf_counter()
    ms = MeanShift(bandwidth=bw, cluster_all=True, n_jobs=-1, seeds=None).fit(X)
    return ms.labels_.astype(np.int64), np.asarray(ms.cluster_centers_, dtype=np.float64), int(ms.n_iter_), time.perf_counter() - t0


def main():
    assert sklearn.__version__ == '1.7.2', sklearn.__version__
    out = {'scenes': np.array(sorted(SCENES))}
    for name, (make, bw) in SCENES.items():
        X = make()
        assert X.dtype == np.float32 and X.shape[1] == 3
        assert name != 'streamed' or len(X) == F64_LDS_POINTS + 4
        stop = 1e-3 * bw
        l32, c32, it32, t32 = run(X, bw)
        l64, c64, it64, t64 = run(X.astype(np.float64), bw)
        assert np.array_equal(l32, l64) and it32 == it64, f'{name}: condition 1'
        assert c32.shape == c64.shape and np.abs(c32 - c64).max() < 0.1 * stop, f'{name}: condition 2 ({np.abs(c32 - c64).max():.3g})'
        margin = np.inf
        if len(c64) > 1:
            d = np.sort(np.linalg.norm(X.astype(np.float64)[:, None] - c64[None], axis=2), axis=1)
            margin = float((d[:, 1] - d[:, 0]).min())
            assert margin >= 50 * stop, f'{name}: condition 3 ({margin:.3g})'
        ref = meanshift_ref.mean_shift(X, bw)
        assert np.array_equal(ref['labels'], l64) and ref['n_iter'] == it64, f'{name}: the restatement disagrees with scikit-learn'
        k = np.sort(ref['center_counts'])
        assert len(k) < 2 or np.diff(k).min() >= 5, f'{name}: condition 4 ({k})'
        print(f'{name}: n {len(X)} centers {len(c64)} n_iter {it64} f32/f64 center gap {np.abs(c32 - c64).max():.3g} m '
              f'margin {margin:.3g} m intensities {ref["center_counts"]} sklearn {t32:.2f} s (f32) {t64:.2f} s (f64)')
        out.update({f'{name}_X': X, f'{name}_bandwidth': np.float64(bw), f'{name}_labels_f32': l32, f'{name}_centers_f32': c32,
                    f'{name}_n_iter_f32': np.int64(it32), f'{name}_labels_f64': l64, f'{name}_centers_f64': c64,
                    f'{name}_n_iter_f64': np.int64(it64)})
    tmp = OUT + '.tmp.npz'
    np.savez_compressed(tmp, **out)
    largest = max(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE) if f.endswith(('.npz', '.pkl')) and 'meanshift' not in f)
    if os.path.getsize(tmp) > largest:
        os.remove(tmp)
        raise AssertionError('condition 5: the file would be larger than the largest committed golden')
    os.replace(tmp, OUT)
    print(OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
