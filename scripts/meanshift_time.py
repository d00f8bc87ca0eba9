"""dev: time of catgrasp_amd.cluster.MeanShift on the golden scenes and on a 16k-point synthetic bin -> profiles/meanshift_time.json.

  python scripts/meanshift_time.py            on the MI355X: HIP-event times of the whole fit and of its stages (climb, both routes where
                                              the cloud fits in LDS; sort and merge; labels), median of --reps after a warm-up
  python scripts/meanshift_time.py --host     on a CPU host with scikit-learn: wall time of sklearn.cluster.MeanShift(n_jobs=-1).fit
                                              on the same inputs

Each mode rewrites its own key of the JSON file and leaves the other.  The two are times of different machines: a device time
and a host time, not a speed-up measured on one system."""
import argparse
import json
import os
import platform
import statistics
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, 'profiles', 'meanshift_time.json')
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'meanshift_golden.npz')
SCENES = ('tiny', 'nut', 'screw', 'touching', 'streamed')


def bin16k():
    """16,384 points: 12 objects of unequal size on a 3 cm grid, spread (3, 1.5, 1.5) mm like the `nut` scene, bandwidth 0.007."""
    rng = np.random.default_rng(16)
    sizes = np.array([2100, 1900, 1750, 1600, 1500, 1400, 1300, 1200, 1100, 1000, 900, 634])
    assert sizes.sum() == 16384
    centers = np.array([[(i % 4) * 0.03, (i // 4) * 0.03, 0.6] for i in range(len(sizes))]) + rng.normal(0, 0.002, (len(sizes), 3))
    pts = np.concatenate([c + rng.normal(0, 1, (n, 3)) * (0.003, 0.0015, 0.0015) for c, n in zip(centers, sizes)])
    return rng.permutation(pts).astype(np.float32), 0.007


def inputs():
    with np.load(GOLDEN) as z:
        cases = {s: (z[f'{s}_X'], float(z[f'{s}_bandwidth'])) for s in SCENES}
    cases['bin16k'] = bin16k()
    return cases


def device_times(reps):
    import torch
    from catgrasp_amd import cluster
    dev = torch.device('cuda:0')

    def timed(fn):
        fn(); torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); out = fn(); b.record(); torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return statistics.median(ms), out

    res = {}
    for name, (X, bw) in inputs().items():
        pts = torch.from_numpy(X).to(dev)
        seeds = pts.double().contiguous()
        row = {'n': len(X), 'bandwidth': bw}
        fits_lds = len(X) * 12 <= 160 * 1024
        for route in (('lds', 'streamed') if fits_lds else ('streamed',)):
            row[f'climb_{route}_ms'], (means, counts, iters) = timed(lambda: cluster.climb(pts, seeds, bw, route=route))
        row['sort_merge_ms'], centers = timed(lambda: cluster.merge(cluster.sort_centers(means, counts), bw))
        row['labels_ms'], _ = timed(lambda: cluster.nearest_center(pts, centers))
        row['fit_ms'], ms = timed(lambda: cluster.MeanShift(bw).fit(pts))            # device tensor in; numpy labels and centers out
        row.update(centers=len(ms.cluster_centers_), n_iter=ms.n_iter_, converged_centers_before_merge=int((counts > 0).sum()))
        res[name] = row
        print(name, row, flush=True)
    return {'device': torch.cuda.get_device_name(0), 'reps': reps, 'timer': 'HIP events, median', 'scenes': res}


def host_times():
    import sklearn
    from sklearn.cluster import MeanShift
    res = {}
    cases = inputs()
    MeanShift(bandwidth=cases['tiny'][1], n_jobs=-1).fit(cases['tiny'][0])         # starts the worker pool: not part of a fit
    for name, (X, bw) in cases.items():
        t0 = time.perf_counter()
        ms = MeanShift(bandwidth=bw, cluster_all=True, n_jobs=-1, seeds=None).fit(X)
        res[name] = {'n': len(X), 'bandwidth': bw, 'fit_s': round(time.perf_counter() - t0, 3), 'centers': len(ms.cluster_centers_), 'n_iter': int(ms.n_iter_)}
        print(name, res[name], flush=True)
    return {'library': f'scikit-learn {sklearn.__version__}, n_jobs=-1', 'cpus': os.cpu_count(), 'machine': platform.machine(),
            'timer': 'wall clock, one run after the worker pool is up', 'scenes': res}


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--host', action='store_true')
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=OUT)
    args = ap.parse_args()
    data = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            data = json.load(f)
    if args.host:
        data['sklearn_on_cpu_host_development_machine'] = host_times()
    else:
        data['catgrasp_amd_on_mi355x'] = device_times(args.reps)
    with open(args.out, 'w') as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write('\n')
