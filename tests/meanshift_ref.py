"""Float64 numpy restatement of mean shift with a flat kernel, written from scikit-learn's documented algorithm
(MeanShift.fit / _mean_shift_single_seed): brute-force radius queries, the same stop rule, the same ordered merge.
It states the arithmetic the device kernels are held to (catgrasp_amd/csrc/meanshift.hip):

  membership   dx*dx + dy*dy + dz*dz <= bandwidth*bandwidth, all float64, from the exact point coordinates
  mean         sum of the members / count, float64 (only the ORDER of the sum is free: numpy's here, lane-strided on the device)
  stop         no member -> empty seed;  |mean - old mean| <= 1e-3 * bandwidth, or completed == max_iter;  else completed += 1
  merge        centers sorted by (count, (x, y, z)) descending; walking them, a live center is kept and kills every center within
               `bandwidth` of it (<=)
  labels       nearest kept center, first minimum

`golden()` is the recorded scikit-learn 1.7.2 result of every scene (tests/golden/make_golden_meanshift.py); `reference(name)` runs
the restatement on a scene once per process, for every test that compares against it.
"""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'meanshift_golden.npz')


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def scenes():
    return [str(s) for s in golden()['scenes']]


def scene(name):
    """-> (X float32, bandwidth)"""
    return golden()[f'{name}_X'], float(golden()[f'{name}_bandwidth'])


@functools.lru_cache(maxsize=None)
def reference(name):
    return mean_shift(*scene(name))


def climb(X, seeds, bandwidth, max_iter=300, chunk=512):
    """-> means (m,3) f64, counts (m) int64, iters (m) int64 of every seed."""
    P = np.asarray(X, dtype=np.float64)
    mean = np.array(seeds, dtype=np.float64)
    m = mean.shape[0]
    bw2, stop = np.float64(bandwidth) * np.float64(bandwidth), 1e-3 * np.float64(bandwidth)
    counts, iters = np.zeros(m, dtype=np.int64), np.zeros(m, dtype=np.int64)
    active = np.arange(m)
    px, py, pz = P[:, 0][None, :], P[:, 1][None, :], P[:, 2][None, :]
    while active.size:
        still = []
        for a in range(0, active.size, chunk):
            ids = active[a:a + chunk]
            mu = mean[ids]
            dx, dy, dz = px - mu[:, 0:1], py - mu[:, 1:2], pz - mu[:, 2:3]
            inside = dx * dx + dy * dy + dz * dz <= bw2
            c = inside.sum(axis=1)
            counts[ids] = c
            has = c > 0                                     # an empty seed stops with the mean it had
            new = mu.copy()
            new[has] = (inside[has].astype(np.float64) @ P) / c[has, None]
            step = np.sqrt(((new - mu) ** 2).sum(axis=1))
            mean[ids] = new
            go = has & ~((step <= stop) | (iters[ids] == max_iter))
            iters[ids[go]] += 1
            still.append(ids[go])
        active = np.concatenate(still)
    return mean, counts, iters


def merge(means, counts, bandwidth):
    """-> the kept centers (k,3) in scikit-learn's order, and their counts."""
    bw2 = np.float64(bandwidth) * np.float64(bandwidth)
    items = sorted({tuple(mu): int(c) for mu, c in zip(means, counts) if c > 0}.items(), key=lambda t: (t[1], t[0]), reverse=True)
    if not items:
        raise ValueError('no seed has a point within the bandwidth')
    C = np.array([t[0] for t in items], dtype=np.float64)
    alive = np.ones(len(C), dtype=bool)
    kept = []
    for i in range(len(C)):
        if alive[i]:
            d = C - C[i]
            alive &= ~(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2] <= bw2)
            kept.append(i)
    return C[kept], np.array([items[i][1] for i in kept], dtype=np.int64)


def nearest(X, centers):
    """Index of the nearest center (first minimum) and the distance."""
    P = np.asarray(X, dtype=np.float64)
    d = P[:, None, :] - centers[None, :, :]
    d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
    idx = d2.argmin(axis=1)
    return idx, np.sqrt(d2[np.arange(len(P)), idx])


def mean_shift(X, bandwidth, seeds=None, max_iter=300, cluster_all=True):
    """-> dict(means, counts, iters per seed; centers, labels, n_iter)."""
    means, counts, iters = climb(X, X if seeds is None else seeds, bandwidth, max_iter)
    centers, center_counts = merge(means, counts, bandwidth)
    labels, dist = nearest(X, centers)
    if not cluster_all:
        labels = np.where(dist <= bandwidth, labels, -1)
    return {'means': means, 'counts': counts, 'iters': iters, 'centers': centers, 'center_counts': center_counts, 'labels': labels.astype(np.int64), 'n_iter': int(iters.max())}
